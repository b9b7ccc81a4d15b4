#!/usr/bin/env python3
"""What a binding-energy evaluation costs (include/agbnp_hip.h: agbnp_hip_binding_execute_device / _energy_device, DESIGN.md
s.4n), beside what a caller could write before it existed, and that adding it has left the full evaluation alone.

(a) In one child process per system: microseconds per BindingEnergy.execute_device() and .energy_device() call, and per call of
    the BASELINE in the same process -- three contexts (complex, receptor, ligand), torch indexing for the gather, execute_group
    (energy_group), torch indexing for the weighted scatter and the two scalars, the members' buffers cleared with torch.  The
    baseline is not gated on the three verdicts (nothing a caller had could do that without a host read): it is the cheapest
    thing a caller could write, not an equivalent.  `--evaluations` calls are enqueued on ONE stream of the caller's at one
    geometry with one synchronise at the end, the kinds alternating over `--repeats` repeats.  Also the launch counts of the
    binding's members: scalars 16, 18 and 19.
(b) With --parent-library (a libagbnp_hip.so built from the parent commit): execute_device() of this build and of the parent's,
    each in a fresh child process, alternating, `--repeats` processes each (the children are scripts/decompose_timing.py's, which
    measure exactly that through the C ABI); each side's mean and its run-to-run spread (max - min).
Version 1, NoCutoff, Reference mode, lambda = 0.35; every figure is a host clock around work that ends in a synchronise.  This
process only starts the children.  Prints tables and one JSON line with the library's build id.

  python scripts/binding_timing.py [--evaluations 2000] [--repeats 5] [--parent-library PATH [--parent-repeats 5]]
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
KINDS = ("binding_execute", "baseline_execute", "binding_energy", "baseline_energy")
LAMBDA = 0.35


def timed_calls(name, evaluations, repeats):
    import numpy as np
    import torch

    import openmm_agbnp_plugin_amd as P

    s = P.load_system(name)
    first, last = SYSTEMS[name]
    ligand = np.arange(first, last + 1)
    receptor = np.setdiff1d(np.arange(s.n), ligand)
    binding = P.BindingEnergy(P.AGBNPForce.from_arrays(*s.params(), version=1), ligand)
    kernels = []
    for sub in (s, s.subset(receptor), s.subset(ligand)):
        k = P.HipCalcAGBNPForceKernel(device=0)
        k.initialize(P.AGBNPForce.from_arrays(*sub.params(), version=1))
        kernels.append(k)
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream()  # (torch's default stream has the handle 0, which the library takes for a context's own stream)
    stream = side.cuda_stream
    f64 = dict(dtype=torch.float64, device=dev)
    pos = torch.tensor(s.pos, **f64).contiguous()
    frc, scalars = torch.zeros((s.n, 3), **f64), torch.zeros(2, **f64)
    idx = [None, torch.tensor(receptor, device=dev), torch.tensor(ligand, device=dev)]
    m_pos = [pos, torch.zeros((len(receptor), 3), **f64), torch.zeros((len(ligand), 3), **f64)]
    m_frc = [torch.zeros_like(p) for p in m_pos]
    m_ene = torch.zeros(3, **f64)
    ptrs = lambda tensors: [t.data_ptr() for t in tensors]  # noqa: E731
    e_ptrs = [m_ene[i:i + 1].data_ptr() for i in range(3)]
    weights = torch.tensor([[LAMBDA, 1.0 - LAMBDA, 1.0 - LAMBDA], [1.0, -1.0, -1.0]], **f64)  # E_lambda and u from (E_RL, E_R, E_L)

    def baseline(full):
        for m in (1, 2):
            torch.index_select(pos, 0, idx[m], out=m_pos[m])
        if full:
            P.execute_group(kernels, ptrs(m_pos), ptrs(m_frc), e_ptrs, stream)
            frc.add_(m_frc[0], alpha=LAMBDA)
            for m in (1, 2):
                frc.index_add_(0, idx[m], m_frc[m], alpha=1.0 - LAMBDA)
            for f in m_frc:
                f.zero_()
        else:
            P.energy_group(kernels, ptrs(m_pos), e_ptrs, stream)
        scalars.add_(weights @ m_ene)
        m_ene.zero_()

    call = {
        "binding_execute": lambda: binding.execute_device(pos.data_ptr(), LAMBDA, frc.data_ptr(), scalars[0:1].data_ptr(), scalars[1:2].data_ptr(), stream),
        "binding_energy": lambda: binding.energy_device(pos.data_ptr(), LAMBDA, scalars[0:1].data_ptr(), scalars[1:2].data_ptr(), stream),
        "baseline_execute": lambda: baseline(True),
        "baseline_energy": lambda: baseline(False),
    }

    def finish_all(what):
        if binding.finish(stream) != 0 or any(k.finish(stream) != 0 for k in kernels):
            raise SystemExit(f"{name}: {what} evaluations were withheld")

    binding.execute(s.pos, LAMBDA)  # (settles the capacity variants and the first masks)
    for k, p in zip(kernels, (s.pos, s.pos[receptor], s.pos[ligand])):
        k.execute(p, np.zeros((len(p), 3)))
    torch.cuda.synchronize()
    out = {kind: [] for kind in KINDS}
    with torch.cuda.stream(side):
        for kind in KINDS:  # warm-up: every kernel of every kind has run
            for _ in range(20):
                call[kind]()
        torch.cuda.synchronize()
        finish_all("warm-up")
        check = {}
        for kind in ("binding_execute", "baseline_execute"):  # the two must compute the same thing
            frc.zero_()
            scalars.zero_()
            call[kind]()
            torch.cuda.synchronize()
            check[kind] = (frc.cpu().numpy().copy(), scalars.cpu().numpy().copy())
        finish_all("check")
        agree = float(np.abs(check["binding_execute"][0] - check["baseline_execute"][0]).max()), float(
            np.abs(check["binding_execute"][1] - check["baseline_execute"][1]).max())
        for _ in range(repeats):
            for kind in KINDS:
                torch.cuda.synchronize()
                start = time.perf_counter()
                for _ in range(evaluations):
                    call[kind]()
                torch.cuda.synchronize()
                out[kind].append(1e6 * (time.perf_counter() - start) / evaluations)
                finish_all(kind)
        binding.execute_device(pos.data_ptr(), LAMBDA, frc.data_ptr(), None, None, stream)
        full = [[int(binding.member(m).scalar(name_)) for name_ in ("launches", "energy_only_launches", "group_members")] for m in range(3)]
        binding.energy_device(pos.data_ptr(), LAMBDA, scalars[0:1].data_ptr(), None, stream)
        shared_energy = [int(binding.member(m).scalar("group_members")) for m in range(3)]
        finish_all("closing")
    return dict(atoms=int(s.n), ligand_atoms=int(len(ligand)), figures=out, binding_and_baseline_differ_by=agree,
                member_scalars_16_18_19=full, energy_group_members=shared_energy)


def cell(v):
    return f"{sum(v) / len(v):.1f} (spread {max(v) - min(v):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--evaluations", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--systems", default=",".join(SYSTEMS))
    ap.add_argument("--parent-library", default=None)
    ap.add_argument("--parent-repeats", type=int, default=None, help="processes per side of part (b); default: --repeats")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)  # one system's figures as a JSON line
    args = ap.parse_args()
    if args.child:
        from openmm_agbnp_plugin_amd import _lib

        got = timed_calls(args.child, args.evaluations, args.repeats)
        got["build_id"] = _lib.build_id()
        print(json.dumps(got))
        return

    def child(script, extra, library=None):
        env = dict(os.environ)
        env.pop("AGBNP_HIP_LIBRARY", None)
        if library:
            env["AGBNP_HIP_LIBRARY"] = os.path.abspath(library)
        done = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script)] + extra + ["--evaluations", str(args.evaluations)],
                              env=env, capture_output=True, text=True, timeout=900)
        if done.returncode != 0:
            raise SystemExit(f"{script} {extra}: child ended with {done.returncode}\n{done.stdout[-1000:]}\n{done.stderr[-2000:]}")
        return json.loads(done.stdout.strip().splitlines()[-1])

    out = {"build_id": None, "evaluations": args.evaluations, "lambda": LAMBDA, "results": []}
    print("| system | atoms (ligand) | binding execute, us | baseline execute, us | binding energy, us | baseline energy, us |")
    print("|---|---|---|---|---|---|")
    for name in args.systems.split(","):
        got = child("binding_timing.py", ["--child", name, "--repeats", str(args.repeats)])
        out["build_id"] = got.pop("build_id")
        f = got["figures"]
        out["results"].append(dict(system=name, **got))
        print(f"| {name} | {got['atoms']} ({got['ligand_atoms']}) | " + " | ".join(cell(f[kind]) for kind in KINDS) + " |", flush=True)
        print(f"  members' scalars 16, 18, 19 (complex, receptor, ligand): {got['member_scalars_16_18_19']}; energy-only call, scalar 19: "
              f"{got['energy_group_members']}; binding and baseline differ by {got['binding_and_baseline_differ_by']}", flush=True)
    if args.parent_library:
        print()
        print("| system | execute_device, this build, us | execute_device, parent build, us |")
        print("|---|---|---|")
        for name in args.systems.split(","):
            sides, builds = {"new": [], "parent": []}, {}
            for _ in range(args.parent_repeats or args.repeats):
                for side, library in (("new", None), ("parent", args.parent_library)):
                    got = child("decompose_timing.py", ["--child", name, "--kinds", "execute", "--repeats", "1"], library)
                    sides[side] += got["figures"]["execute"]
                    builds[side] = got["build_id"]
            out["results"].append(dict(system=name, execute_us=sides["new"], parent_execute_us=sides["parent"], parent_build_id=builds["parent"]))
            print(f"| {name} | {cell(sides['new'])} | {cell(sides['parent'])} |", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
