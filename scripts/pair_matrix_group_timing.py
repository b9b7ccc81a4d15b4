#!/usr/bin/env python3
"""What pair-matrix groups and the set-pair matrix of a binding energy cost (include/agbnp_hip.h: agbnp_hip_pair_matrix_group,
agbnp_hip_binding_pair_matrix_device), beside what a caller could write before they existed, and that adding
them has left the full evaluation alone.

(a) One child process per group size: microseconds per pair_matrix_group() call over R trpcage contexts with the residue
    partition, and per round of the same members' R pair_matrix_device() calls back to back, in the same process.
(b) One child process per system: microseconds per BindingEnergy.pair_matrix_device() call, and per call of the BASELINE in the
    same process -- three contexts (complex, receptor, ligand) with the partition restricted by hand, two index_select calls for
    the gather, three pair_matrix_device calls, the subtraction in torch, the members' matrices cleared with torch.  The baseline
    is not gated on the three verdicts (nothing a caller had could do that without a host read): the cheapest thing a caller
    could write, not an equivalent.  Also the members' scalars 18, 19 and 20 behind a binding matrix: 1 + 5 + 1 launches where
    scalar 19 is 3.
(c) With --parent-library (a libagbnp_hip.so built from the parent commit): execute_device() of this build and of the parent's,
    each in a fresh child process, alternating, `--repeats` processes each (the children are scripts/decompose_timing.py's,
    which measure exactly that through the C ABI); each side's mean and its run-to-run spread (max - min).
`--evaluations` calls are enqueued on ONE stream of the caller's at one geometry per member with one synchronise per figure, the
kinds alternating over `--repeats` repeats.  Version 1, NoCutoff, Reference mode; every figure is a host clock around work that
ends in a synchronise.  This process only starts the children.  Prints tables and one JSON line with the library's build id.

  python scripts/pair_matrix_group_timing.py [--evaluations 2000] [--repeats 5] [--sizes 4,8] [--systems trpcage,1dwc]
                                             [--parent-library PATH [--parent-repeats 5]]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from decompose_group_timing import SYSTEMS, cell, timed  # noqa: E402  (the same clock and the same ligands)


def residues(name):
    import openmm_agbnp_plugin_amd as P

    sets, labels = P.load_sets(os.path.join(ROOT, "tests", "golden", f"residues_{name}.txt"))
    return sets, len(labels)


def group_calls(members, evaluations, repeats):
    import numpy as np
    import torch

    import openmm_agbnp_plugin_amd as P

    s = P.load_system("trpcage")
    sets, S = residues("trpcage")
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream()  # (torch's default stream has the handle 0, which the library takes for a context's own stream)
    stream = side.cuda_stream
    f64 = dict(dtype=torch.float64, device=dev)
    kernels = []
    for m in range(members):
        k = P.HipCalcAGBNPForceKernel(device=0)
        k.initialize(P.AGBNPForce.from_arrays(*s.params(), version=1))
        k.set_atom_sets(sets, S)
        k.execute(s.jittered(m), np.zeros((s.n, 3)))  # (settles the capacity variant and the first masks)
        kernels.append(k)
    pos = [torch.tensor(s.jittered(m), **f64).contiguous() for m in range(members)]
    mats = [torch.zeros((S, S), **f64) for _ in range(members)]
    ene = torch.zeros(members, **f64)
    p_pos, p_mats = [t.data_ptr() for t in pos], [t.data_ptr() for t in mats]
    p_ene = [ene[m:m + 1].data_ptr() for m in range(members)]

    def alone():
        for k, a, b, c in zip(kernels, p_pos, p_mats, p_ene):
            k.pair_matrix_device(a, b, c, stream)

    def finish_all(what):
        if any(k.finish(stream) != 0 for k in kernels):
            raise SystemExit(f"{members} members: {what} evaluations were withheld")

    call = {"group": lambda: P.pair_matrix_group(kernels, p_pos, p_mats, p_ene, stream), "alone": alone}
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out = timed(call, ("group", "alone"), evaluations, repeats, finish_all)
        check = {}
        for kind in ("group", "alone"):  # the two must compute the same thing
            for t in mats:
                t.zero_()
            call[kind]()
            torch.cuda.synchronize()
            check[kind] = np.stack([t.cpu().numpy() for t in mats])
        call["group"]()
        scalars = [[int(k.scalar(name)) for name in ("energy_only_launches", "group_members", "last_evaluation_kind")] for k in kernels]
        finish_all("closing")
    return dict(members=members, atoms=int(s.n), sets=S, figures=out,
                group_and_alone_differ_by=float(np.abs(check["group"] - check["alone"]).max()), member_scalars_18_19_20=scalars)


def binding_calls(name, evaluations, repeats):
    import numpy as np
    import torch

    import openmm_agbnp_plugin_amd as P

    s = P.load_system(name)
    sets, S = residues(name)
    first, last = SYSTEMS[name]
    ligand = np.arange(first, last + 1)
    receptor = np.setdiff1d(np.arange(s.n), ligand)
    binding = P.BindingEnergy(P.AGBNPForce.from_arrays(*s.params(), version=1), ligand)
    binding.set_atom_sets(sets, S)
    kernels = []
    for sub, own in ((s, sets), (s.subset(receptor), sets[receptor]), (s.subset(ligand), sets[ligand])):
        k = P.HipCalcAGBNPForceKernel(device=0)
        k.initialize(P.AGBNPForce.from_arrays(*sub.params(), version=1))
        k.set_atom_sets(own, S)
        kernels.append(k)
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream()
    stream = side.cuda_stream
    f64 = dict(dtype=torch.float64, device=dev)
    pos = torch.tensor(s.pos, **f64).contiguous()
    d, u = torch.zeros((S, S), **f64), torch.zeros(1, **f64)
    idx = [None, torch.tensor(receptor, device=dev), torch.tensor(ligand, device=dev)]
    m_pos = [pos, torch.zeros((len(receptor), 3), **f64), torch.zeros((len(ligand), 3), **f64)]
    m_mats = torch.zeros((3, S, S), **f64)
    m_ene = torch.zeros(3, **f64)
    weights = torch.tensor([1.0, -1.0, -1.0], **f64)  # u from (E_RL, E_R, E_L), D from the three matrices

    def baseline():
        for m in (1, 2):
            torch.index_select(pos, 0, idx[m], out=m_pos[m])
        for m, k in enumerate(kernels):
            k.pair_matrix_device(m_pos[m].data_ptr(), m_mats[m].data_ptr(), m_ene[m:m + 1].data_ptr(), stream)
        d.add_(m_mats[0] - m_mats[1] - m_mats[2])
        u.add_(weights @ m_ene)
        m_mats.zero_()
        m_ene.zero_()

    call = {"binding": lambda: binding.pair_matrix_device(pos.data_ptr(), d.data_ptr(), u.data_ptr(), stream), "baseline": baseline}

    def finish_all(what):
        if binding.finish(stream) != 0 or any(k.finish(stream) != 0 for k in kernels):
            raise SystemExit(f"{name}: {what} evaluations were withheld")

    binding.pair_matrix(s.pos)  # (settles the capacity variants and the first masks)
    for k, p in zip(kernels, (s.pos, s.pos[receptor], s.pos[ligand])):
        k.execute(p, np.zeros((len(p), 3)))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out = timed(call, ("binding", "baseline"), evaluations, repeats, finish_all)
        check = {}
        for kind in ("binding", "baseline"):  # the two must compute the same thing
            d.zero_()
            u.zero_()
            call[kind]()
            torch.cuda.synchronize()
            check[kind] = (d.cpu().numpy().copy(), u.item())
        finish_all("check")
        agree = float(np.abs(check["binding"][0] - check["baseline"][0]).max()), abs(check["binding"][1] - check["baseline"][1])
        call["binding"]()
        scalars = [[int(binding.member(m).scalar(x)) for x in ("energy_only_launches", "group_members", "last_evaluation_kind")] for m in range(3)]
        finish_all("closing")
    return dict(atoms=int(s.n), ligand_atoms=int(len(ligand)), sets=S, figures=out, binding_and_baseline_differ_by=agree,
                member_scalars_18_19_20=scalars, u=check["binding"][1], matrix_sum=float(check["binding"][0].sum()))


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
    print("| trpcage members | pair_matrix_group, us per call | the members' pair_matrix_device calls, us per round | per member: group / alone |")
    print("|---|---|---|---|")
    for size in [x for x in args.sizes.split(",") if x]:
        got = child("pair_matrix_group_timing.py", ["--child", f"group:{size}", "--repeats", str(args.repeats)])
        out["build_id"] = got.pop("build_id")
        f, r = got["figures"], got["members"]
        out["results"].append(dict(kind="group", **got))
        mean = {k: sum(v) / len(v) for k, v in f.items()}
        print(f"| {r} | {cell(f['group'])} | {cell(f['alone'])} | {mean['group'] / r:.1f} / {mean['alone'] / r:.1f} |", flush=True)
        print(f"  {got['sets']} sets; members' scalars 18, 19, 20: {got['member_scalars_18_19_20'][0]} (all alike: "
              f"{all(x == got['member_scalars_18_19_20'][0] for x in got['member_scalars_18_19_20'])}); group and alone differ by "
              f"{got['group_and_alone_differ_by']}", flush=True)
    print()
    print("| system | atoms (ligand), sets | binding pair_matrix_device, us | baseline, us |")
    print("|---|---|---|---|")
    for name in [x for x in args.systems.split(",") if x]:
        got = child("pair_matrix_group_timing.py", ["--child", f"binding:{name}", "--repeats", str(args.repeats)])
        out["build_id"] = got.pop("build_id")
        f = got["figures"]
        out["results"].append(dict(kind="binding", system=name, **got))
        print(f"| {name} | {got['atoms']} ({got['ligand_atoms']}), {got['sets']} | {cell(f['binding'])} | {cell(f['baseline'])} |", flush=True)
        print(f"  members' scalars 18, 19, 20 (complex, receptor, ligand): {got['member_scalars_18_19_20']}; binding and baseline differ by "
              f"{got['binding_and_baseline_differ_by']}; u = {got['u']:.6f}, the matrix sums to {got['matrix_sum']:.6f}", flush=True)
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
