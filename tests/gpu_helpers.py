"""What several GPU test files share word for word: tolerances, the fixtures that pin the five-launch mode, comparisons, device
buffers of a group's members.  A plain module: the test files import what they use (helpers that differ between files stay there)."""
import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P

TIGHT = 1e-7
SAME = 1e-9


@pytest.fixture()
def five(monkeypatch):
    monkeypatch.setenv("AGBNP_HIP_FIVE_LAUNCHES", "1")


@pytest.fixture()
def five_groups(monkeypatch):
    """The group tests' `five`: shared launches at their default as well."""
    monkeypatch.setenv("AGBNP_HIP_FIVE_LAUNCHES", "1")
    monkeypatch.delenv("AGBNP_HIP_GROUP_LAUNCHES", raising=False)


def kernel_of(params, version=1, mode="reference"):
    k = P.HipCalcAGBNPForceKernel(device=0, mode=mode)
    k.initialize(P.AGBNPForce.from_arrays(*params, version=version))
    return k


def freeze_packing(k, nheavy, per_forest=8):
    """A packing frozen from the host (test hook agbnp_debug_set_packing): forest f = the whole subtrees of heavy atoms
    per_forest f .. per_forest f + per_forest - 1, whatever their size.  `k`: a kernel, or the view of a binding's member
    (BindingEnergy.member()): anything with the context's handle in _h.  Returns the number of forests."""
    import ctypes as C

    from openmm_agbnp_plugin_amd import _lib
    lib = _lib.load()
    lib.agbnp_debug_set_packing.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int]
    nf = (nheavy + per_forest - 1) // per_forest
    order = (C.c_int * nheavy)(*range(nheavy))
    start = (C.c_int * (nf + 1))(*[min(per_forest * f, nheavy) for f in range(nf + 1)])
    assert lib.agbnp_debug_set_packing(k._h, order, nheavy, start, nf, 1) == _lib.OK
    return nf


def energy_close(e, eo, tol=TIGHT):
    assert abs(e - eo) < tol * max(1.0, abs(eo) * 1e-3), f"energy differs by {abs(e - eo):.3e}"


def close(e, f, eo, fo, tol=TIGHT):
    energy_close(e, eo, tol)
    assert np.abs(f - fo).max() < tol, f"forces differ by {np.abs(f - fo).max():.3e}"


class Buffers:
    """Device positions, forces and energy of one member (torch tensors)."""

    def __init__(self, torch, n):
        dev = torch.device("cuda:0")
        self.torch = torch
        self.pos = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        self.frc = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        self.ene = torch.zeros((1,), dtype=torch.float64, device=dev)

    def load(self, geom, fill=0.0):
        self.pos.copy_(self.torch.tensor(geom, dtype=self.torch.float64))
        self.frc.fill_(fill)
        self.ene.zero_()

    def ptrs(self):
        return self.pos.data_ptr(), self.frc.data_ptr(), self.ene.data_ptr()

    def result(self):
        return self.ene.item(), self.frc.cpu().numpy()


def execute_group(kernels, bufs, stream):
    P.execute_group(kernels, [b.pos.data_ptr() for b in bufs], [b.frc.data_ptr() for b in bufs], [b.ene.data_ptr() for b in bufs],
                    stream)


def cluster(n, spacing, seed):
    """A cluster denser than a protein (as tests/test_gpu_parity.py builds them): its subtrees need the larger LDS variants."""
    from openmm_agbnp_plugin_amd.systems import vdw_alpha_from_radius
    rng = np.random.default_rng(seed)
    grid = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
    pos = grid * spacing + rng.normal(0, 0.02, (n, 3))
    ish = (rng.random(n) < 0.3).astype(np.int32)
    radius = np.where(ish == 1, 0.121, rng.choice([0.17, 0.18, 0.19, 0.2], n))
    gamma = np.where(ish == 1, 0.0, 0.117 * 418.4)
    return P.AGBNPSystem(f"cluster{spacing}_{seed}", pos, radius, gamma, vdw_alpha_from_radius(radius), rng.normal(0, 0.4, n), ish)
