"""An OpenMM GPU context's buffers, as agbnp_hip_execute_openmm reads and writes them (include/agbnp_hip.h; the conventions of the
reference's OpenCL platform, OpenCLAGBNPKernels.cpp:541-556): a shuffled atom index padded to a multiple of 32, posq in the context's
order (double4; float4 + correction; float4 alone), the 2^32 fixed-point force planes [x | y | z], the energy buffer.  What
tests/test_gpu_five_launches.py::test_the_openmm_entry_point_runs_in_the_mode builds inline, for the tests that drive that entry point.
A plain module like tests/gpu_helpers.py: the test files import what they use."""
import os

import numpy as np

from tests.gpu_helpers import TIGHT

ENERGY_SLOT = 3
FIXED_POINT = 1e-6  # per accumulated evaluation: the fixed point resolves 2^-32 per add
STEPS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "protocol_steps.dat")


def protocol_geometries(pos):
    """The evaluations of the repeat-protocol sequence (tests/golden/protocol_steps.dat): the geometry of evaluation k and the atoms
    stage k moved, k = 0 .. 3."""
    stages = {}
    for line in open(STEPS):
        if line.strip() and not line.startswith("#"):
            stage, atom, dx, dy, dz = line.split()
            stages.setdefault(int(stage), []).append((int(atom), np.array([float(dx), float(dy), float(dz)])))
    geoms, moved = [np.array(pos, dtype=np.float64)], [[]]
    for stage in sorted(stages):
        g = geoms[-1].copy()
        for atom, d in stages[stage]:
            g[atom] += d
        geoms.append(g)
        moved.append(stages[stage])
    return geoms, moved


class OpenMMContext:
    """`oracle` is evaluated at the positions the engine really sees: the caller's (double), hi + lo (mixed), the float-rounded ones
    (single)."""

    def __init__(self, torch, n, precision, oracle, seed=11):
        assert precision in ("double", "mixed", "single")
        self.torch, self.n, self.precision, self.oracle = torch, n, precision, oracle
        self.padded = (n + 31) // 32 * 32
        self.dev = torch.device("cuda:0")
        self.rng = np.random.default_rng(seed)
        self.index = torch.zeros(self.padded, dtype=torch.int32, device=self.dev)
        self.fixed = torch.zeros(3 * self.padded, dtype=torch.int64, device=self.dev)
        self.energy_is_double = precision != "single"
        self.ebuf = torch.zeros(8, dtype=torch.float64 if self.energy_is_double else torch.float32, device=self.dev)
        # one posq (+ correction) whose ADDRESS stays, for evaluations captured into a graph: load() copies new contents in
        real = torch.float64 if precision == "double" else torch.float32
        self.posq = torch.zeros((self.padded, 4), dtype=real, device=self.dev)
        self.corr = torch.zeros((self.padded, 4), dtype=torch.float32, device=self.dev) if precision == "mixed" else None
        self.order = None
        self.reorder()

    def reorder(self):
        """OpenMM's reorderAtoms(): the same index array, new contents."""
        self.order = self.rng.permutation(self.n).astype(np.int32)
        full = np.concatenate([self.order, np.arange(self.n, self.padded, dtype=np.int32)])
        self.index.copy_(self.torch.tensor(full))
        self.torch.cuda.synchronize()

    def host_arrays(self, pos):
        """-> posq, correction (or None) as host arrays in the context's order, and the positions the engine sees [n, 3]."""
        host = np.zeros((self.padded, 4))
        host[: self.n, :3] = pos[self.order]
        if self.precision == "double":
            return host, None, np.array(pos, dtype=np.float64)
        hi = host.astype(np.float32)
        lo = (host - hi.astype(np.float64)).astype(np.float32) if self.precision == "mixed" else None
        seen = np.zeros((self.n, 3))
        seen[self.order] = (hi.astype(np.float64) + (lo.astype(np.float64) if lo is not None else 0.0))[: self.n, :3]
        return hi, lo, seen

    def load(self, pos):
        """New contents for the resident posq (+ correction); returns the positions the engine sees."""
        hi, lo, seen = self.host_arrays(pos)
        self.posq.copy_(self.torch.tensor(hi))
        if lo is not None:
            self.corr.copy_(self.torch.tensor(lo))
        return seen

    def enqueue(self, kernel, posq=None, corr=None, stream=None):
        """One agbnp_hip_execute_openmm on the resident posq (or on the tensors given)."""
        posq = self.posq if posq is None else posq
        corr = self.corr if posq is self.posq else corr
        stream = self.torch.cuda.current_stream().cuda_stream if stream is None else stream
        kernel.execute_openmm(posq.data_ptr(), self.precision == "double", corr.data_ptr() if corr is not None else 0, self.index.data_ptr(),
                              self.padded, self.fixed.data_ptr(), self.ebuf.data_ptr(), self.energy_is_double, ENERGY_SLOT, stream)

    def run(self, kernel, geoms, expect=True):
        """Queues one evaluation per geometry (each on arrays of its own, kept alive in the first return value); returns the
        oracle's sums at the positions the engine sees (expect=False: zeros -- evaluations nobody compares, settling ones)."""
        keep, want_e, want_f = [], 0.0, np.zeros((self.n, 3))
        for g in geoms:
            hi, lo, seen = self.host_arrays(g)
            posq = self.torch.tensor(hi, device=self.dev)
            corr = self.torch.tensor(lo, device=self.dev) if lo is not None else None
            keep.append((posq, corr))
            self.enqueue(kernel, posq, corr)
            if expect:
                eo, fo = self.oracle.execute(seen)
                want_e, want_f = want_e + eo, want_f + fo
        return keep, want_e, want_f

    def expected(self, geoms):
        """The oracle's sums over `geoms` at the positions the engine sees."""
        want = [self.oracle.execute(self.host_arrays(g)[2]) for g in geoms]
        return sum(w[0] for w in want), sum(w[1] for w in want)

    def forces(self):
        """The fixed-point planes as forces in PARTICLE order [n, 3]; the padding slots must be untouched."""
        self.torch.cuda.synchronize()
        got = self.fixed.cpu().numpy().reshape(3, self.padded).astype(np.float64) / 2.0 ** 32
        assert not got[:, self.n:].any()
        out = np.zeros((self.n, 3))
        out[self.order] = got[:, : self.n].T
        return out

    def energy(self):
        self.torch.cuda.synchronize()
        e = self.ebuf.cpu().numpy().astype(np.float64)
        assert not np.delete(e, ENERGY_SLOT).any()
        return float(e[ENERGY_SLOT])

    def untouched(self):
        self.torch.cuda.synchronize()
        return not self.fixed.cpu().numpy().any() and not self.ebuf.cpu().numpy().any()

    def clear(self):
        self.fixed.zero_()
        self.ebuf.zero_()

    def check(self, want_e, want_f, evaluations, what=""):
        """The buffers against the oracle's sums of `evaluations` accumulated evaluations, at the tolerances of
        test_the_openmm_entry_point_runs_in_the_mode; prints the deviations first, clears the buffers, returns (|dE|, max|dF|).
        (single: a float accumulator holds seven digits of the energy -- the forces alone are compared.)"""
        df = float(np.abs(self.forces() - want_f).max())
        de = abs(self.energy() - want_e)
        print(f"{what or 'openmm entry'}: {evaluations} evaluation(s)  |dE|={de:.3e}  max|dF|={df:.3e}")
        assert df < evaluations * FIXED_POINT
        if self.energy_is_double:
            assert de < evaluations * TIGHT * max(1.0, abs(want_e) * 1e-3 / evaluations)
        self.clear()
        return de, df
