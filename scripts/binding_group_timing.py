#!/usr/bin/env python3
"""What a binding group costs (include/agbnp_hip.h: agbnp_hip_binding_execute_group / _energy_group) beside the
same bindings evaluated one call after another, what a step and an exchange attempt of BindingReplicaMD cost, and that adding
them has left the single-binding call and the plain evaluation alone.

(a) Group against back-to-back, one child process per system and K (1, 4, 5, 6, 8, 16): K bindings of one complex, binding k at
    jittered(k % 4), lambdas even from 0 to 1.  Microseconds per binding-evaluation of the group call and of K
    agbnp_hip_binding_execute_device calls in the same process, and the same for the energy-only forms; `--evaluations` rounds
    are enqueued on ONE stream of the caller's with one synchronise at the end, the kinds alternating over `--repeats` repeats.
    Also scalar 19 of the first binding's members.
(b) Driver, one child process per R (4, 8): milliseconds per Langevin step of BindingReplicaMD between attempts (a run without
    exchanges) and per attempt (a run with an attempt after every step, minus the steps).
(c) With --parent-library (a libagbnp_hip.so built from the parent commit): agbnp_hip_binding_execute_device and
    agbnp_hip_execute_device of this build and of the parent's through the C ABI alone, each in a fresh child process,
    alternating, `--repeats` processes each; each side's mean and its run-to-run spread (max - min).
Version 1, NoCutoff, Reference mode; every figure is a host clock around work that ends in a synchronise.  This process only
starts the children.  Prints tables and one JSON line with the library's build id.

  python scripts/binding_group_timing.py [--evaluations 2000] [--repeats 5] [--systems trpcage,1dwc] [--sizes 1,4,5,6,8,16]
                                         [--parent-library PATH]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SYSTEMS = {"trpcage": (0, 15), "1dwc": (4122, 4151)}  # system -> first and last ligand atom
SIZES = (1, 4, 5, 6, 8, 16)
KINDS = ("group_execute", "single_execute", "group_energy", "single_energy")


def timed_group(name, count, evaluations, repeats):
    import numpy as np
    import torch

    import openmm_agbnp_plugin_amd as P

    s = P.load_system(name)
    first, last = SYSTEMS[name]
    ligand = np.arange(first, last + 1)
    bindings = [P.BindingEnergy(P.AGBNPForce.from_arrays(*s.params(), version=1), ligand) for _ in range(count)]
    lams = np.linspace(0.0, 1.0, count) if count > 1 else np.array([0.35])
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream()  # (torch's default stream has the handle 0, which the library takes for a context's own stream)
    stream = side.cuda_stream
    f64 = dict(dtype=torch.float64, device=dev)
    geoms = [s.jittered(k % 4) for k in range(count)]
    pos = [torch.tensor(g, **f64).contiguous() for g in geoms]
    frc = [torch.zeros((s.n, 3), **f64) for _ in range(count)]
    scalars = torch.zeros((count, 2), **f64)
    lam = torch.tensor(lams, **f64)
    ptrs = lambda tensors: [t.data_ptr() for t in tensors]  # noqa: E731
    p_pos, p_frc = ptrs(pos), ptrs(frc)
    p_e, p_u = [scalars[k, 0:1].data_ptr() for k in range(count)], [scalars[k, 1:2].data_ptr() for k in range(count)]

    def single(full):
        for k, b in enumerate(bindings):
            if full:
                b.execute_device(p_pos[k], float(lams[k]), p_frc[k], p_e[k], p_u[k], stream)
            else:
                b.energy_device(p_pos[k], float(lams[k]), p_e[k], p_u[k], stream)

    call = {
        "group_execute": lambda: P.binding_execute_group(bindings, p_pos, lam.data_ptr(), p_frc, p_e, p_u, stream),
        "group_energy": lambda: P.binding_energy_group(bindings, p_pos, lam.data_ptr(), p_e, p_u, stream),
        "single_execute": lambda: single(True),
        "single_energy": lambda: single(False),
    }

    def finish_all(what):
        if any(b.finish(stream) != 0 for b in bindings):
            raise SystemExit(f"{name} K = {count}: {what} evaluations were withheld")

    for b, g in zip(bindings, geoms):
        b.execute(g, 0.35)  # (settles the capacity variants and the first masks)
    torch.cuda.synchronize()
    out = {kind: [] for kind in KINDS}
    with torch.cuda.stream(side):
        for kind in KINDS:  # warm-up: every kernel of every kind has run
            for _ in range(20):
                call[kind]()
        torch.cuda.synchronize()
        finish_all("warm-up")
        check = {}
        for kind in ("group_execute", "single_execute"):  # the two must compute the same thing
            for f in frc:
                f.zero_()
            scalars.zero_()
            call[kind]()
            torch.cuda.synchronize()
            check[kind] = (np.stack([f.cpu().numpy() for f in frc]), scalars.cpu().numpy().copy())
        finish_all("check")
        agree = [float(np.abs(check["group_execute"][j] - check["single_execute"][j]).max()) for j in range(2)]
        for _ in range(repeats):
            for kind in KINDS:
                torch.cuda.synchronize()
                start = time.perf_counter()
                for _ in range(evaluations):
                    call[kind]()
                torch.cuda.synchronize()
                out[kind].append(1e6 * (time.perf_counter() - start) / (evaluations * count))
                finish_all(kind)
        call["group_execute"]()
        shared = [int(bindings[0].member(m).scalar("group_members")) for m in range(3)]
        finish_all("closing")
    return dict(atoms=int(s.n), ligand_atoms=int(len(ligand)), bindings=count, figures=out, group_and_single_differ_by=agree, scalar_19=shared)


def timed_driver(name, replicas, steps):
    import numpy as np
    import torch

    import openmm_agbnp_plugin_amd as P
    from openmm_agbnp_plugin_amd.md import BindingReplicaMD

    s = P.load_system(name)
    first, last = SYSTEMS[name]
    ligand = np.arange(first, last + 1)
    bindings = [P.BindingEnergy(P.AGBNPForce.from_arrays(*s.params(), version=1), ligand) for _ in range(replicas)]
    md = BindingReplicaMD(s, bindings, np.linspace(0.0, 1.0, replicas), 300.0, k_tether=1.0e5)
    md.settle()
    md.forces()
    md.finish()
    md.run(20, "langevin", exchange_every=1, check_every=20)

    def clock(exchange_every):
        torch.cuda.synchronize()
        start = time.perf_counter()
        missed = md.run(steps, "langevin", exchange_every=exchange_every, check_every=steps)
        torch.cuda.synchronize()
        if missed.any():
            raise SystemExit(f"{name} R = {replicas}: evaluations were withheld")
        return 1e3 * (time.perf_counter() - start) / steps

    plain = [clock(0) for _ in range(3)]
    every = [clock(1) for _ in range(3)]
    log = md.exchange_log()
    return dict(atoms=int(s.n), replicas=replicas, ms_per_step=plain, ms_per_attempt=[a - min(plain) for a in every],
                void_pairs=int((log["accepted"] < 0).sum()), pairs=int(len(log)), acceptance=[float(a) for a in md.acceptance()])


def timed_existing(name, library, evaluations):
    """[us per agbnp_hip_binding_execute_device call], [us per agbnp_hip_execute_device call] through the C ABI alone (the symbols
    that the parent's library has too), for part (c)."""
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
    lib.agbnp_hip_binding_create.argtypes = [C.POINTER(vp), C.c_int, dp, dp, dp, dp, ip, ip, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int]
    lib.agbnp_hip_binding_execute_host.argtypes = [vp, dp, C.c_double, dp, dp, dp]
    lib.agbnp_hip_binding_execute_device.argtypes = [vp, vp, C.c_double, vp, vp, vp, vp]
    lib.agbnp_hip_binding_finish.argtypes = [vp, vp, ip]
    lib.agbnp_hip_binding_destroy.argtypes = [vp]
    lib.agbnp_hip_build_id.restype = C.c_char_p
    s = P.load_system(name)
    first, last = SYSTEMS[name]
    ligand = np.arange(first, last + 1, dtype=np.int32)
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in s.params()[:4]] + [np.ascontiguousarray(s.ishydrogen, dtype=np.int32)]
    params = [a.ctypes.data_as(dp) for a in arrays[:4]] + [arrays[4].ctypes.data_as(ip)]
    h, b = vp(), vp()
    if lib.agbnp_hip_create(C.byref(h), s.n, *params, 1, 0, 1.0, 0) != 0:
        raise SystemExit(f"{name}: agbnp_hip_create failed")
    if lib.agbnp_hip_binding_create(C.byref(b), s.n, *params, ligand.ctypes.data_as(ip), len(ligand), 1, 0, 1.0, 0) != 0:
        raise SystemExit(f"{name}: agbnp_hip_binding_create failed")
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream()
    stream = vp(side.cuda_stream)
    pos = torch.tensor(s.pos, dtype=torch.float64, device=dev).contiguous()
    frc = torch.zeros((s.n, 3), dtype=torch.float64, device=dev)
    ene = torch.zeros((2,), dtype=torch.float64, device=dev)
    hpos, hfrc, e, u, rep = np.ascontiguousarray(s.pos, dtype=np.float64), np.zeros((s.n, 3)), C.c_double(0.0), C.c_double(0.0), C.c_int(0)
    lib.agbnp_hip_execute_host(h, hpos.ctypes.data_as(dp), hfrc.ctypes.data_as(dp), C.byref(e))
    lib.agbnp_hip_binding_execute_host(b, hpos.ctypes.data_as(dp), 0.35, hfrc.ctypes.data_as(dp), C.byref(e), C.byref(u))
    torch.cuda.synchronize()
    figures = {"binding_execute": [], "execute": []}
    calls = {
        "binding_execute": lambda: lib.agbnp_hip_binding_execute_device(b, vp(pos.data_ptr()), 0.35, vp(frc.data_ptr()), vp(ene.data_ptr()),
                                                                        vp(ene[1:2].data_ptr()), stream),
        "execute": lambda: lib.agbnp_hip_execute_device(h, vp(pos.data_ptr()), vp(frc.data_ptr()), vp(ene.data_ptr()), stream),
    }
    finish = {"binding_execute": lambda: lib.agbnp_hip_binding_finish(b, stream, C.byref(rep)),
              "execute": lambda: lib.agbnp_hip_finish(h, stream, C.byref(rep))}
    for kind in figures:
        for timed in (False, True):  # (the first round is the warm-up)
            torch.cuda.synchronize()
            start = time.perf_counter()
            for _ in range(evaluations if timed else 20):
                if calls[kind]() != 0:
                    raise SystemExit(f"{name}: {kind} failed")
            torch.cuda.synchronize()
            if timed:
                figures[kind].append(1e6 * (time.perf_counter() - start) / evaluations)
            if finish[kind]() != 0 or rep.value != 0:
                raise SystemExit(f"{name}: {kind} evaluations were withheld")
    build = lib.agbnp_hip_build_id().decode()
    lib.agbnp_hip_binding_destroy(b)
    lib.agbnp_hip_destroy(h)
    return dict(atoms=int(s.n), figures=figures, build_id=build)


def cell(v, digits=1):
    return f"{sum(v) / len(v):.{digits}f} (spread {max(v) - min(v):.{digits}f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--evaluations", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--systems", default=",".join(SYSTEMS))
    ap.add_argument("--sizes", default=",".join(str(k) for k in SIZES))
    ap.add_argument("--driver-replicas", default="4,8")
    ap.add_argument("--driver-steps", type=int, default=500)
    ap.add_argument("--parent-library", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)  # group | driver | existing: one row as a JSON line
    ap.add_argument("--system", default="trpcage", help=argparse.SUPPRESS)
    ap.add_argument("--count", type=int, default=1, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        from openmm_agbnp_plugin_amd import _lib

        if args.child == "group":
            got = timed_group(args.system, args.count, args.evaluations, args.repeats)
        elif args.child == "driver":
            got = timed_driver(args.system, args.count, args.driver_steps)
        else:
            got = timed_existing(args.system, os.environ.get("AGBNP_HIP_LIBRARY") or _lib.LIB_PATH, args.evaluations)
        got.setdefault("build_id", _lib.build_id() if args.child != "existing" else None)
        print(json.dumps(got))
        return

    def child(kind, system, count=1, library=None):
        env = dict(os.environ)
        env.pop("AGBNP_HIP_LIBRARY", None)
        if library:
            env["AGBNP_HIP_LIBRARY"] = os.path.abspath(library)
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--system", system, "--count", str(count),
                               "--evaluations", str(args.evaluations), "--repeats", str(args.repeats), "--driver-steps", str(args.driver_steps)],
                              env=env, capture_output=True, text=True, timeout=900)
        if done.returncode != 0:
            raise SystemExit(f"{kind} {system} {count}: child ended with {done.returncode}\n{done.stdout[-1000:]}\n{done.stderr[-2000:]}")
        return json.loads(done.stdout.strip().splitlines()[-1])

    systems = args.systems.split(",")
    out = {"build_id": None, "evaluations": args.evaluations, "results": []}
    print("| system | K | group execute, us | back-to-back execute, us | group energy, us | back-to-back energy, us | scalar 19 |")
    print("|---|---|---|---|---|---|---|")
    for name in systems:
        for count in [int(k) for k in args.sizes.split(",") if k]:
            got = child("group", name, count)
            out["build_id"] = got.pop("build_id")
            out["results"].append(dict(system=name, **got))
            f = got["figures"]
            print(f"| {name} | {count} | " + " | ".join(cell(f[kind]) for kind in KINDS) + f" | {got['scalar_19']} |", flush=True)
    print()
    print("| system | R | ms per step between attempts | ms per attempt | void pairs |")
    print("|---|---|---|---|---|")
    for name in systems:
        for replicas in [int(r) for r in args.driver_replicas.split(",") if r]:
            got = child("driver", name, replicas)
            got.pop("build_id")
            out["results"].append(dict(system=name, **got))
            print(f"| {name} | {replicas} | {cell(got['ms_per_step'], 4)} | {cell(got['ms_per_attempt'], 4)} | {got['void_pairs']} of {got['pairs']} |", flush=True)
    if args.parent_library:
        print()
        print("| system | binding execute_device: this build, us | parent build, us | execute_device: this build, us | parent build, us |")
        print("|---|---|---|---|---|")
        for name in systems:
            sides = {side: {"binding_execute": [], "execute": []} for side in ("new", "parent")}
            builds = {}
            for _ in range(args.repeats):
                for side, library in (("new", None), ("parent", args.parent_library)):
                    got = child("existing", name, library=library)
                    for kind in sides[side]:
                        sides[side][kind] += got["figures"][kind]
                    builds[side] = got["build_id"]
            out["results"].append(dict(system=name, existing=sides, build_ids=builds))
            print(f"| {name} | {cell(sides['new']['binding_execute'])} | {cell(sides['parent']['binding_execute'])} | "
                  f"{cell(sides['new']['execute'])} | {cell(sides['parent']['execute'])} |", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
