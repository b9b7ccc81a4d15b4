#!/usr/bin/env python3
"""What decomposition groups and the per-atom decomposition of a binding energy cost (include/agbnp_hip.h:
agbnp_hip_decompose_group, agbnp_hip_binding_decompose_device), beside what a caller could write before they
existed, and that adding them has left the full evaluation alone.

(a) One child process per group size: microseconds per decompose_group() call over R trpcage contexts, and per round of the same
    members' R decompose_device() calls back to back, in the same process.
(b) One child process per system: microseconds per BindingEnergy.decompose_device() call, and per call of the BASELINE in the
    same process -- three contexts (complex, receptor, ligand), two index_select calls for the gather, three decompose_device
    calls, the scatter and the subtraction in torch, the members' planes cleared with torch.  The baseline is not gated on the
    three verdicts (nothing a caller had could do that without a host read): the cheapest thing a caller could write, not an
    equivalent.  Also the members' scalars 18, 19 and 20 behind a binding decomposition: 1 + 5 + 1 launches where scalar 19 is 3.
(c) With --parent-library (a libagbnp_hip.so built from the parent commit): execute_device() of this build and of the parent's,
    each in a fresh child process, alternating, `--repeats` processes each (the children are scripts/decompose_timing.py's,
    which measure exactly that through the C ABI); each side's mean and its run-to-run spread (max - min).
`--evaluations` calls are enqueued on ONE stream of the caller's at one geometry per member with one synchronise per figure, the
kinds alternating over `--repeats` repeats.  Version 1, NoCutoff, Reference mode; every figure is a host clock around work that
ends in a synchronise.  This process only starts the children.  Prints tables and one JSON line with the library's build id.

  python scripts/decompose_group_timing.py [--evaluations 2000] [--repeats 5] [--sizes 4,8] [--systems trpcage,1dwc]
                                           [--parent-library PATH [--parent-repeats 5]]
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


def timed(call, kinds, evaluations, repeats, finish_all):
    import torch

    out = {kind: [] for kind in kinds}
    for kind in kinds:  # warm-up: every kernel of every kind has run
        for _ in range(20):
            call[kind]()
    torch.cuda.synchronize()
    finish_all("warm-up")
    for _ in range(repeats):
        for kind in kinds:
            torch.cuda.synchronize()
            start = time.perf_counter()
            for _ in range(evaluations):
                call[kind]()
            torch.cuda.synchronize()
            out[kind].append(1e6 * (time.perf_counter() - start) / evaluations)
            finish_all(kind)
    return out


def group_calls(members, evaluations, repeats):
    import numpy as np
    import torch

    import openmm_agbnp_plugin_amd as P

    s = P.load_system("trpcage")
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream()  # (torch's default stream has the handle 0, which the library takes for a context's own stream)
    stream = side.cuda_stream
    f64 = dict(dtype=torch.float64, device=dev)
    kernels = []
    for m in range(members):
        k = P.HipCalcAGBNPForceKernel(device=0)
        k.initialize(P.AGBNPForce.from_arrays(*s.params(), version=1))
        k.execute(s.jittered(m), np.zeros((s.n, 3)))  # (settles the capacity variant and the first masks)
        kernels.append(k)
    pos = [torch.tensor(s.jittered(m), **f64).contiguous() for m in range(members)]
    planes = [torch.zeros((4, s.n), **f64) for _ in range(members)]
    ene = torch.zeros(members, **f64)
    p_pos, p_planes = [t.data_ptr() for t in pos], [t.data_ptr() for t in planes]
    p_ene = [ene[m:m + 1].data_ptr() for m in range(members)]

    def alone():
        for k, a, b, c in zip(kernels, p_pos, p_planes, p_ene):
            k.decompose_device(a, b, c, stream)

    def finish_all(what):
        if any(k.finish(stream) != 0 for k in kernels):
            raise SystemExit(f"{members} members: {what} evaluations were withheld")

    call = {"group": lambda: P.decompose_group(kernels, p_pos, p_planes, p_ene, stream), "alone": alone}
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out = timed(call, ("group", "alone"), evaluations, repeats, finish_all)
        check = {}
        for kind in ("group", "alone"):  # the two must compute the same thing
            for t in planes:
                t.zero_()
            call[kind]()
            torch.cuda.synchronize()
            check[kind] = np.stack([t.cpu().numpy() for t in planes])
        call["group"]()
        scalars = [[int(k.scalar(name)) for name in ("energy_only_launches", "group_members", "last_evaluation_kind")] for k in kernels]
        finish_all("closing")
    return dict(members=members, atoms=int(s.n), figures=out, group_and_alone_differ_by=float(np.abs(check["group"] - check["alone"]).max()),
                member_scalars_18_19_20=scalars)


def binding_calls(name, evaluations, repeats):
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
    side = torch.cuda.Stream()
    stream = side.cuda_stream
    f64 = dict(dtype=torch.float64, device=dev)
    pos = torch.tensor(s.pos, **f64).contiguous()
    terms, u = torch.zeros((4, s.n), **f64), torch.zeros(1, **f64)
    idx = [None, torch.tensor(receptor, device=dev), torch.tensor(ligand, device=dev)]
    m_pos = [pos, torch.zeros((len(receptor), 3), **f64), torch.zeros((len(ligand), 3), **f64)]
    m_terms = [torch.zeros((4, len(p)), **f64) for p in m_pos]
    m_ene = torch.zeros(3, **f64)
    weights = torch.tensor([1.0, -1.0, -1.0], **f64)  # u from (E_RL, E_R, E_L)

    def baseline():
        for m in (1, 2):
            torch.index_select(pos, 0, idx[m], out=m_pos[m])
        for m, k in enumerate(kernels):
            k.decompose_device(m_pos[m].data_ptr(), m_terms[m].data_ptr(), m_ene[m:m + 1].data_ptr(), stream)
        terms.add_(m_terms[0])
        for m in (1, 2):
            terms.index_add_(1, idx[m], m_terms[m], alpha=-1.0)
        u.add_(weights @ m_ene)
        for t in m_terms:
            t.zero_()
        m_ene.zero_()

    call = {"binding": lambda: binding.decompose_device(pos.data_ptr(), terms.data_ptr(), u.data_ptr(), stream), "baseline": baseline}

    def finish_all(what):
        if binding.finish(stream) != 0 or any(k.finish(stream) != 0 for k in kernels):
            raise SystemExit(f"{name}: {what} evaluations were withheld")

    binding.decompose(s.pos)  # (settles the capacity variants and the first masks)
    for k, p in zip(kernels, (s.pos, s.pos[receptor], s.pos[ligand])):
        k.execute(p, np.zeros((len(p), 3)))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out = timed(call, ("binding", "baseline"), evaluations, repeats, finish_all)
        check = {}
        for kind in ("binding", "baseline"):  # the two must compute the same thing
            terms.zero_()
            u.zero_()
            call[kind]()
            torch.cuda.synchronize()
            check[kind] = (terms.cpu().numpy().copy(), u.item())
        finish_all("check")
        agree = float(np.abs(check["binding"][0] - check["baseline"][0]).max()), abs(check["binding"][1] - check["baseline"][1])
        call["binding"]()
        scalars = [[int(binding.member(m).scalar(x)) for x in ("energy_only_launches", "group_members", "last_evaluation_kind")] for m in range(3)]
        finish_all("closing")
    return dict(atoms=int(s.n), ligand_atoms=int(len(ligand)), figures=out, binding_and_baseline_differ_by=agree,
                member_scalars_18_19_20=scalars, u=check["binding"][1], plane_totals=[float(x) for x in check["binding"][0].sum(axis=1)])


def cell(v):
    return f"{sum(v) / len(v):.1f} (spread {max(v) - min(v):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--evaluations", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="4,8")
    ap.add_argument("--systems", default=",".join(SYSTEMS))
    ap.add_argument("--parent-library", default=None)
    ap.add_argument("--parent-repeats", type=int, default=None, help="processes per side of part (c); default: --repeats")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)  # "group:R" or "binding:SYSTEM": one row's figures as a JSON line
    args = ap.parse_args()
    if args.child:
        from openmm_agbnp_plugin_amd import _lib

        what, which = args.child.split(":")
        got = group_calls(int(which), args.evaluations, args.repeats) if what == "group" else binding_calls(which, args.evaluations, args.repeats)
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

    out = {"build_id": None, "evaluations": args.evaluations, "results": []}
    print("| trpcage members | decompose_group, us per call | the members' decompose_device calls, us per round | per member: group / alone |")
    print("|---|---|---|---|")
    for size in [x for x in args.sizes.split(",") if x]:
        got = child("decompose_group_timing.py", ["--child", f"group:{size}", "--repeats", str(args.repeats)])
        out["build_id"] = got.pop("build_id")
        f, r = got["figures"], got["members"]
        out["results"].append(dict(kind="group", **got))
        mean = {k: sum(v) / len(v) for k, v in f.items()}
        print(f"| {r} | {cell(f['group'])} | {cell(f['alone'])} | {mean['group'] / r:.1f} / {mean['alone'] / r:.1f} |", flush=True)
        print(f"  members' scalars 18, 19, 20: {got['member_scalars_18_19_20'][0]} (all alike: "
              f"{all(x == got['member_scalars_18_19_20'][0] for x in got['member_scalars_18_19_20'])}); group and alone differ by "
              f"{got['group_and_alone_differ_by']}", flush=True)
    print()
    print("| system | atoms (ligand) | binding decompose_device, us | baseline, us |")
    print("|---|---|---|---|")
    for name in [x for x in args.systems.split(",") if x]:
        got = child("decompose_group_timing.py", ["--child", f"binding:{name}", "--repeats", str(args.repeats)])
        out["build_id"] = got.pop("build_id")
        f = got["figures"]
        out["results"].append(dict(kind="binding", system=name, **got))
        print(f"| {name} | {got['atoms']} ({got['ligand_atoms']}) | {cell(f['binding'])} | {cell(f['baseline'])} |", flush=True)
        print(f"  members' scalars 18, 19, 20 (complex, receptor, ligand): {got['member_scalars_18_19_20']}; binding and baseline differ by "
              f"{got['binding_and_baseline_differ_by']}; u = {got['u']:.6f}, plane totals {got['plane_totals']}", flush=True)
    if args.parent_library:
        print()
        print("| system | execute_device, this build, us | execute_device, parent build, us |")
        print("|---|---|---|")
        for name in [x for x in args.systems.split(",") if x]:
            sides, builds = {"new": [], "parent": []}, {}
            for _ in range(args.parent_repeats or args.repeats):
                for side, library in (("new", None), ("parent", args.parent_library)):
                    got = child("decompose_timing.py", ["--child", name, "--kinds", "execute", "--repeats", "1"], library)
                    sides[side] += got["figures"]["execute"]
                    builds[side] = got["build_id"]
            out["results"].append(dict(kind="parent", system=name, execute_us=sides["new"], parent_execute_us=sides["parent"],
                                       parent_build_id=builds["parent"]))
            print(f"| {name} | {cell(sides['new'])} | {cell(sides['parent'])} |", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
