"""What the analysis-group timing scripts share (decompose_group_timing.py, pair_matrix_group_timing.py): the clock, the child
processes, the set-up and the checks of their parts (a) and (b), part (c) and main().  A script hands in its KIND, a class made
once per system (`Kind(name)`) that says what differs between the analyses:

  group, device, host        the names of the group call (of the package) and of a kernel's / a binding's device and host calls
  GROUP_HEADER, BINDING_HEADER   the two tables' header lines
  keys                       the result keys of its own that are known before anything runs ({} or the number of sets)
  partition(obj, atoms=None) sets its partition, restricted to `atoms`, on a kernel or a binding (nothing where there is none)
  shape(n)                   the shape of the output of a system of n atoms
  members(sizes, f64)        the baseline's three member outputs;  combine(out, members, idx) adds them to `out`, in torch, and clears them
  result_keys(D)             the result keys of its own that are read off a binding's output
  group_note(got), binding_cell(got), binding_note(got)   what its table rows say beyond the common columns
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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


def cell(v):
    return f"{sum(v) / len(v):.1f} (spread {max(v) - min(v):.1f})"


def run_child(script, extra, evaluations, library=None, timeout=900):
    """One figure's fresh process: scripts/`script` with `extra` and --evaluations; `library` is its AGBNP_HIP_LIBRARY (None:
    the tree's own).  Returns the JSON line it ends with."""
    env = dict(os.environ)
    env.pop("AGBNP_HIP_LIBRARY", None)
    if library:
        env["AGBNP_HIP_LIBRARY"] = os.path.abspath(library)
    done = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script)] + extra + ["--evaluations", str(evaluations)],
                          env=env, capture_output=True, text=True, timeout=timeout)
    if done.returncode != 0:
        raise SystemExit(f"{script} {extra}: child ended with {done.returncode}\n{done.stdout[-1000:]}\n{done.stderr[-2000:]}")
    return json.loads(done.stdout.strip().splitlines()[-1])


def measure(side, call, outputs, evaluations, repeats, finish_all, read, members):
    """With `side` torch's stream: the figures of both kinds of `call`, then one call of each on cleared outputs (read(): what
    the two must agree on), then one more of the first kind and the scalars 18, 19 and 20 of `members` behind it."""
    import torch

    kinds = tuple(call)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        figures = timed(call, kinds, evaluations, repeats, finish_all)
        check = {}
        for kind in kinds:  # the two must compute the same thing
            for t in outputs:
                t.zero_()
            call[kind]()
            torch.cuda.synchronize()
            check[kind] = read()
        finish_all("check")
        call[kinds[0]]()
        scalars = [[int(k.scalar(name)) for name in ("energy_only_launches", "group_members", "last_evaluation_kind")] for k in members]
        finish_all("closing")
    return figures, check, scalars


def group_calls(Kind, members, evaluations, repeats):
    import numpy as np
    import torch

    import openmm_agbnp_plugin_amd as P

    s, kind = P.load_system("trpcage"), Kind("trpcage")
    side = torch.cuda.Stream()  # (torch's default stream has the handle 0, which the library takes for a context's own stream)
    stream = side.cuda_stream
    f64 = dict(dtype=torch.float64, device=torch.device("cuda:0"))
    kernels = []
    for m in range(members):
        k = P.HipCalcAGBNPForceKernel(device=0)
        k.initialize(P.AGBNPForce.from_arrays(*s.params(), version=1))
        kind.partition(k)
        k.execute(s.jittered(m), np.zeros((s.n, 3)))  # (settles the capacity variant and the first masks)
        kernels.append(k)
    pos = [torch.tensor(s.jittered(m), **f64).contiguous() for m in range(members)]
    outs = [torch.zeros(kind.shape(s.n), **f64) for _ in range(members)]
    ene = torch.zeros(members, **f64)
    p_pos, p_outs = [t.data_ptr() for t in pos], [t.data_ptr() for t in outs]
    p_ene = [ene[m:m + 1].data_ptr() for m in range(members)]

    def alone():
        for k, a, b, c in zip(kernels, p_pos, p_outs, p_ene):
            getattr(k, kind.device)(a, b, c, stream)

    def finish_all(what):
        if any(k.finish(stream) != 0 for k in kernels):
            raise SystemExit(f"{members} members: {what} evaluations were withheld")

    call = {"group": lambda: getattr(P, kind.group)(kernels, p_pos, p_outs, p_ene, stream), "alone": alone}
    figures, check, scalars = measure(side, call, outs, evaluations, repeats, finish_all, lambda: np.stack([t.cpu().numpy() for t in outs]),
                                      kernels)
    return dict(members=members, atoms=int(s.n), **kind.keys, figures=figures,
                group_and_alone_differ_by=float(np.abs(check["group"] - check["alone"]).max()), member_scalars_18_19_20=scalars)


def binding_calls(Kind, name, evaluations, repeats):
    import numpy as np
    import torch

    import openmm_agbnp_plugin_amd as P

    s, kind = P.load_system(name), Kind(name)
    first, last = SYSTEMS[name]
    ligand = np.arange(first, last + 1)
    receptor = np.setdiff1d(np.arange(s.n), ligand)
    binding = P.BindingEnergy(P.AGBNPForce.from_arrays(*s.params(), version=1), ligand)
    kind.partition(binding)
    kernels = []
    for sub, atoms in ((s, None), (s.subset(receptor), receptor), (s.subset(ligand), ligand)):
        k = P.HipCalcAGBNPForceKernel(device=0)
        k.initialize(P.AGBNPForce.from_arrays(*sub.params(), version=1))
        kind.partition(k, atoms)
        kernels.append(k)
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream()
    stream = side.cuda_stream
    f64 = dict(dtype=torch.float64, device=dev)
    pos = torch.tensor(s.pos, **f64).contiguous()
    d, u = torch.zeros(kind.shape(s.n), **f64), torch.zeros(1, **f64)
    idx = [None, torch.tensor(receptor, device=dev), torch.tensor(ligand, device=dev)]
    m_pos = [pos, torch.zeros((len(receptor), 3), **f64), torch.zeros((len(ligand), 3), **f64)]
    m_outs = kind.members([len(p) for p in m_pos], f64)
    m_ene = torch.zeros(3, **f64)
    weights = torch.tensor([1.0, -1.0, -1.0], **f64)  # u from (E_RL, E_R, E_L)

    def baseline():
        for m in (1, 2):
            torch.index_select(pos, 0, idx[m], out=m_pos[m])
        for m, k in enumerate(kernels):
            getattr(k, kind.device)(m_pos[m].data_ptr(), m_outs[m].data_ptr(), m_ene[m:m + 1].data_ptr(), stream)
        kind.combine(d, m_outs, idx)
        u.add_(weights @ m_ene)
        m_ene.zero_()

    call = {"binding": lambda: getattr(binding, kind.device)(pos.data_ptr(), d.data_ptr(), u.data_ptr(), stream), "baseline": baseline}

    def finish_all(what):
        if binding.finish(stream) != 0 or any(k.finish(stream) != 0 for k in kernels):
            raise SystemExit(f"{name}: {what} evaluations were withheld")

    getattr(binding, kind.host)(s.pos)  # (settles the capacity variants and the first masks)
    for k, p in zip(kernels, (s.pos, s.pos[receptor], s.pos[ligand])):
        k.execute(p, np.zeros((len(p), 3)))
    figures, check, scalars = measure(side, call, (d, u), evaluations, repeats, finish_all, lambda: (d.cpu().numpy().copy(), u.item()),
                                      [binding.member(m) for m in range(3)])
    agree = float(np.abs(check["binding"][0] - check["baseline"][0]).max()), abs(check["binding"][1] - check["baseline"][1])
    return dict(atoms=int(s.n), ligand_atoms=int(len(ligand)), **kind.keys, figures=figures, binding_and_baseline_differ_by=agree,
                member_scalars_18_19_20=scalars, u=check["binding"][1], **kind.result_keys(check["binding"][0]))


def parent_table(systems, parent_library, repeats, evaluations, results):
    """Part (c): execute_device() of this build and of the parent's, alternating fresh scripts/decompose_timing.py children."""
    print()
    print("| system | execute_device, this build, us | execute_device, parent build, us |")
    print("|---|---|---|")
    for name in systems:
        sides, builds = {"new": [], "parent": []}, {}
        for _ in range(repeats):
            for side, library in (("new", None), ("parent", parent_library)):
                got = run_child("decompose_timing.py", ["--child", name, "--kinds", "execute", "--repeats", "1"], evaluations, library)
                sides[side] += got["figures"]["execute"]
                builds[side] = got["build_id"]
        results.append(dict(kind="parent", system=name, execute_us=sides["new"], parent_execute_us=sides["parent"],
                            parent_build_id=builds["parent"]))
        print(f"| {name} | {cell(sides['new'])} | {cell(sides['parent'])} |", flush=True)


def main(script, Kind):
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
        got = (group_calls(Kind, int(which), args.evaluations, args.repeats) if what == "group" else
               binding_calls(Kind, which, args.evaluations, args.repeats))
        got["build_id"] = _lib.build_id()
        print(json.dumps(got))
        return

    def row(which):
        got = run_child(script, ["--child", which, "--repeats", str(args.repeats)], args.evaluations)
        out["build_id"] = got.pop("build_id")
        return got

    out = {"build_id": None, "evaluations": args.evaluations, "results": []}
    systems = [x for x in args.systems.split(",") if x]
    print(Kind.GROUP_HEADER)
    print("|---|---|---|---|")
    for size in [x for x in args.sizes.split(",") if x]:
        got = row(f"group:{size}")
        f, r, scalars = got["figures"], got["members"], got["member_scalars_18_19_20"]
        out["results"].append(dict(kind="group", **got))
        mean = {k: sum(v) / len(v) for k, v in f.items()}
        print(f"| {r} | {cell(f['group'])} | {cell(f['alone'])} | {mean['group'] / r:.1f} / {mean['alone'] / r:.1f} |", flush=True)
        print(f"  {Kind.group_note(got)}members' scalars 18, 19, 20: {scalars[0]} (all alike: {all(x == scalars[0] for x in scalars)}); "
              f"group and alone differ by {got['group_and_alone_differ_by']}", flush=True)
    print()
    print(Kind.BINDING_HEADER)
    print("|---|---|---|---|")
    for name in systems:
        got = row(f"binding:{name}")
        f = got["figures"]
        out["results"].append(dict(kind="binding", system=name, **got))
        print(f"| {name} | {got['atoms']} ({got['ligand_atoms']}){Kind.binding_cell(got)} | {cell(f['binding'])} | {cell(f['baseline'])} |", flush=True)
        print(f"  members' scalars 18, 19, 20 (complex, receptor, ligand): {got['member_scalars_18_19_20']}; binding and baseline differ by "
              f"{got['binding_and_baseline_differ_by']}; u = {got['u']:.6f}, {Kind.binding_note(got)}", flush=True)
    if args.parent_library:
        parent_table(systems, args.parent_library, args.parent_repeats or args.repeats, args.evaluations, out["results"])
    print(json.dumps(out))
