"""CPU: pins tests/binding_decomposition_restatement.py, the reference of the GPU tests of the per-atom decomposition of a
binding energy (tests/test_gpu_binding_decomposition.py): D = T_RL - T_own sums to the binding energy u of
tests/binding_restatement.py, and with the ligand far from the receptor nothing but the screened Coulomb tail of the GB pair
plane is left of it.

Bounds.  The sum: 1e-9 kJ/mol, what tests/test_decomposition_restatement.py holds for its sums (each member's planes sum to its
oracle energy within that; measured here: 4.9e-11 at most).  The separated pair, 5 nm: in version 0 the only term is the cavity
plane, whose overlaps are Gaussians that vanish to FP64 at that distance -- every entry is 0 within 1e-12; in version 1 the Born
radii meet the other body only through descreening integrals inside the 2 nm table reach, so planes 0 to 2 are the same in the
complex as alone (below 1e-6), and plane 3 keeps q_i q_j / d for the pairs that cross the gap: it equals u to 1e-6."""
import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from tests.binding_decomposition_restatement import restate
from tests.binding_restatement import restate as restate_binding

CASES = {  # name -> (system, ligand atoms, version)
    "trpcage_0_15_v1": ("trpcage", range(0, 16), 1),
    "trpcage_100_129_v0": ("trpcage", range(100, 130), 0),
    "fixture264_200_263": ("fixture264", range(200, 264), 1),
}
SEPARATION = 5.0  # nm


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_terms_sum_to_the_binding_energy(name):
    system, ligand, version = CASES[name]
    s = P.load_system(system)
    d, u = restate(s.params(), ligand, s.pos, version=version)
    u_ref = restate_binding(s.params(), ligand, s.pos, 0.35, version=version)[1]
    print(f"{name}: u = {u_ref!r}, |sum D - u| = {abs(d.sum() - u_ref):.3e}, planes {d.sum(axis=1)}")
    assert d.shape == (4, s.n) and np.isfinite(d).all()
    assert u == u_ref
    assert abs(d.sum() - u_ref) < 1e-9
    if version == 0:
        assert (d[1:] == 0.0).all()


def _separated(s, ligand):
    """The ligand translated until its bounding box is SEPARATION away from the receptor's along x."""
    ligand = np.asarray(list(ligand))
    receptor = np.setdiff1d(np.arange(s.n), ligand)
    pos = s.pos.copy()
    pos[ligand, 0] += pos[receptor, 0].max() - pos[ligand, 0].min() + SEPARATION
    return pos


def test_version_0_has_no_term_across_a_gap():
    s = P.load_system("trpcage")
    ligand = range(100, 130)
    d, u = restate(s.params(), ligand, _separated(s, ligand), version=0)
    print(f"version 0, {SEPARATION} nm apart: max |D| = {np.abs(d).max():.3e}, u = {u:.3e}")
    assert np.abs(d).max() < 1e-12
    assert abs(u) < 1e-9  # (a difference of three oracle energies of some 1e3 kJ/mol: the bound of the sums)


def test_version_1_keeps_the_coulomb_tail_in_the_pair_plane():
    s = P.load_system("trpcage")
    ligand = range(0, 16)
    d, u = restate(s.params(), ligand, _separated(s, ligand), version=1)
    print(f"version 1, {SEPARATION} nm apart: max |D[0:3]| = {np.abs(d[:3]).max():.3e}, sum D[3] = {d[3].sum()!r}, u = {u!r}")
    assert np.abs(d[:3]).max() < 1e-6
    assert abs(d[3].sum() - u) < 1e-6
    assert abs(u) > 1e-3  # (the tail is there: a charged ligand 5 nm from a charged receptor)
