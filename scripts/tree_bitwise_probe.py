#!/usr/bin/env python3
"""Forces and energies of the tree stage's larger stores in deterministic mode, for a byte-for-byte comparison of two libraries
(bench.py's systems only reach the 432-node store).  The deterministic mode runs the same tree kernels with TreeArgs::det set,
and its sums do not depend on order, so two builds of the same arithmetic give the same bytes.

  AGBNP_HIP_LIBRARY=<library> python scripts/tree_bitwise_probe.py --out DIR      one library: writes DIR/<case>.npz
  python scripts/tree_bitwise_probe.py --compare DIR_A DIR_B                      exit status 1 unless every case is equal
                                                                                  (force components that are NaN: counted, not compared)

Cases: the three dense clusters of tests/test_gpu_parity.py::test_every_capacity_variant_is_exact (stores of 1024 and 2048
nodes and the HBM-scratch store) with AGBNP_HIP_SPLIT_FIT=0 (every subtree whole) and with the default (big subtrees shared,
forests healed), two geometries each, and the 16 608-atom lattice of 1dwc (more forests than workgroups: the queued replay).
Each case runs in a child process of its own, because the knob is read when a context is created."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLUSTERS = [(150, 0.24, 1), (150, 0.22, 1), (180, 0.18, 2)]  # n, spacing, seed: variants 2, 3, 4 with whole subtrees
CASES = [f"cluster{i}_{fit}" for i in range(len(CLUSTERS)) for fit in ("whole", "default")] + ["lattice"]


def cluster(n, spacing, seed, radii=(0.17, 0.18, 0.19, 0.2), hydrogen_fraction=0.3):  # (as the test makes them)
    import openmm_agbnp_plugin_amd as P
    from openmm_agbnp_plugin_amd.systems import vdw_alpha_from_radius

    rng = np.random.default_rng(seed)
    grid = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
    pos = grid * spacing + rng.normal(0, 0.02, (n, 3))
    ish = (rng.random(n) < hydrogen_fraction).astype(np.int32)
    radius = np.where(ish == 1, 0.121, rng.choice(list(radii), n))
    gamma = np.where(ish == 1, 0.0, 0.117 * 418.4)
    return P.AGBNPSystem(f"cluster{spacing}_{seed}", pos, radius, gamma, vdw_alpha_from_radius(radius), rng.normal(0, 0.4, n), ish)


def run_case(case, out):
    import openmm_agbnp_plugin_amd as P

    if case == "lattice":
        s = P.lattice(P.load_system("1dwc"), 2, 2, 1, 7.0)
        seed = 3
    else:
        i = int(case[len("cluster")])
        s = cluster(*CLUSTERS[i])
        seed = CLUSTERS[i][2] + 100
    geoms = [s.pos, s.pos + np.random.default_rng(seed).normal(0.0, 0.001, s.pos.shape), s.pos]
    k = P.HipCalcAGBNPForceKernel(mode="deterministic")
    k.initialize(P.AGBNPForce.from_arrays(*s.params(), version=1))
    energies, forces = [], []
    for g in geoms:  # (the third evaluation: the first geometry again, on the packing and the variant the others left)
        f = np.zeros((s.n, 3))
        energies.append(k.execute(g, f))
        forces.append(f)
    np.savez(os.path.join(out, case + ".npz"), energy=np.array(energies), forces=np.array(forces),
             variant=int(k.scalar("variant")), forests=int(k.scalar("forests")))
    print(f"{case}: variant {int(k.scalar('variant'))}, {int(k.scalar('forests'))} forests, E = {energies[-1]!r}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--case", help="(child process) one case")
    ap.add_argument("--compare", nargs=2, metavar="DIR")
    args = ap.parse_args()
    if args.compare:
        bad = 0
        for case in CASES:
            a, b = (np.load(os.path.join(d, case + ".npz")) for d in args.compare)
            same = all(a[key].tobytes() == b[key].tobytes() for key in ("energy", "variant", "forests"))
            # (cluster1_default, sharing with a queued replay, returns NaN force components on a different set of atoms in
            # every process, with any library: DESIGN.md s.7.  Only the components that are numbers in both are compared.)
            both = np.isfinite(a["forces"]) & np.isfinite(b["forces"])
            same = same and a["forces"][both].tobytes() == b["forces"][both].tobytes()
            note = "" if both.all() else f"; {both.size - int(both.sum())} of {both.size} force components NaN in one or both, NOT compared"
            print(f"{case}: {'equal byte for byte' if same else 'DIFFERENT'} (variant {int(a['variant'])}, {int(a['forests'])} forests{note})")
            bad += not same
        sys.exit(1 if bad else 0)
    os.makedirs(args.out, exist_ok=True)
    if args.case:
        return run_case(args.case, args.out)
    for case in CASES:
        env = dict(os.environ)
        env.pop("AGBNP_HIP_SPLIT_FIT", None)
        if case.endswith("_whole"):
            env["AGBNP_HIP_SPLIT_FIT"] = "0"
        subprocess.run([sys.executable, os.path.abspath(__file__), "--out", args.out, "--case", case], env=env, check=True, timeout=300)


if __name__ == "__main__":
    main()
