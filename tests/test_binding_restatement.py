"""CPU: pins tests/binding_restatement.py, the reference of the GPU tests of the binding-energy evaluations
(tests/test_gpu_binding.py): the two ends of lambda are the complex's own oracle and the separated pair, E_lambda is linear in
lambda, F_lambda is minus the gradient of E_lambda by central differences, and the partition whose receptor has no heavy atom has
no binding energy in version 0."""
import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from oracle import Oracle
from tests.binding_restatement import BindingRestatement, combine, partition, restate
from tests.edge_systems import edge_systems

CASES = {  # name -> (system, ligand atoms, version)
    "trpcage_0_15": ("trpcage", range(0, 16), 1),
    "fixture264_200_263": ("fixture264", range(200, 264), 1),
}
_cache = {}


def case(name):
    if name not in _cache:
        system, ligand, version = CASES[name]
        s = P.load_system(system)
        r = BindingRestatement(s.params(), ligand, version=version)
        _cache[name] = (s, r, r.evaluate(s.pos))
    return _cache[name]


def test_partition_orders_both_sides_ascending():
    receptor, ligand = partition(10, [7, 2, 9])
    assert ligand.tolist() == [2, 7, 9] and receptor.tolist() == [0, 1, 3, 4, 5, 6, 8]
    for bad in ([], list(range(10)), [3, 3], [10], [-1]):
        with pytest.raises(AssertionError):
            partition(10, bad)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_ends_of_lambda_are_the_complex_and_the_separated_pair(name):
    s, r, (energies, f_rl, f_own) = case(name)
    version = CASES[name][2]
    e1, u, f1 = combine(energies, f_rl, f_own, 1.0)
    eo, fo = Oracle(*s.params(), version=version).execute(s.pos)
    assert e1 == eo and np.array_equal(f1, fo)
    e0, u0, f0 = combine(energies, f_rl, f_own, 0.0)
    sub_r, sub_l = s.subset(r.receptor), s.subset(r.ligand)
    er, fr = Oracle(*sub_r.params(), version=version).execute(sub_r.pos)
    el, fl = Oracle(*sub_l.params(), version=version).execute(sub_l.pos)
    assert e0 == er + el and u0 == u == eo - er - el
    assert np.array_equal(f0[r.receptor], fr) and np.array_equal(f0[r.ligand], fl)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_energy_is_linear_in_lambda_with_slope_u(name):
    _, _, (energies, f_rl, f_own) = case(name)
    e0, u, _ = combine(energies, f_rl, f_own, 0.0)
    for lam in (-0.5, 0.35, 0.5, 1.0, 1.5):
        e, u_lam, f = combine(energies, f_rl, f_own, lam)
        assert u_lam == u
        assert abs(e - (e0 + lam * u)) < 1e-9
        assert np.abs(f - (lam * f_rl + (1.0 - lam) * f_own)).max() < 1e-9


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_force_is_minus_the_gradient_of_the_hybrid_energy(name):
    """Central differences, h = 1e-5 nm, on the first ligand atom, the first receptor atom and the last ligand atom; the bar is
    the project's parity bar, 1e-4 kJ/mol/nm (measured: 2e-6 where forces reach 700)."""
    s, r, (energies, f_rl, f_own) = case(name)
    lam, h = 0.35, 1e-5
    _, _, f = combine(energies, f_rl, f_own, lam)
    worst = 0.0
    for atom in (int(r.ligand[0]), int(r.receptor[0]), int(r.ligand[-1])):
        for d in range(3):
            e = []
            for sign in (1.0, -1.0):
                pos = s.pos.copy()
                pos[atom, d] += sign * h
                e.append(combine(*r.evaluate(pos), lam)[0])
            worst = max(worst, abs(-(e[0] - e[1]) / (2.0 * h) - f[atom, d]))
    print(f"{name}: worst |central difference - F_lambda| = {worst:.2e} kJ/mol/nm")
    assert worst < 1e-4


def test_the_binding_energies_at_the_file_geometries():
    """What the three oracles give for the partitions the GPU tests use, at the bundled coordinates (kJ/mol)."""
    s = P.load_system("trpcage")
    assert abs(restate(s.params(), range(0, 16), s.pos, 0.35, version=1)[1] - 441.642267) < 1e-5
    assert abs(restate(s.params(), range(100, 130), s.pos, 0.35, version=0)[1] - (-69.621371)) < 1e-5
    d = P.load_system("1dwc")
    assert abs(restate(d.params(), range(4122, 4152), d.pos, 0.35, version=1)[1] - 313.305894) < 1e-5


def test_a_receptor_without_heavy_atoms_has_no_version_0_binding_energy():
    """size_1_33 with its one heavy atom as the ligand: the receptor is 32 hydrogens, whose GaussVol energy is 0, and the
    hydrogens do not enter the complex's either."""
    s = edge_systems()["size_1_33"]
    heavy = np.flatnonzero(s.ishydrogen == 0)
    assert len(heavy) == 1
    e_lam, u, f, (e_rl, e_r, e_l) = restate(s.params(), heavy, s.pos, 0.35, version=0)
    assert e_r == 0.0 and abs(u) < 1e-9 and abs(e_lam - e_rl) < 1e-9
    assert np.isfinite(f).all()
