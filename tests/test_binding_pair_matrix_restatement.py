"""CPU: pins tests/binding_pair_matrix_restatement.py, the reference of the GPU tests of the set-pair matrix of a binding energy
(tests/test_gpu_binding_pair_matrix.py): D = M_RL - M_R - M_L is symmetric, sums to the binding energy u, its rows sum to the
per-set sums of the binding's per-atom decomposition (tests/binding_decomposition_restatement.py), a cell between a set wholly in
the receptor and a set wholly in the ligand is the complex's own cell, and version 0 fills the diagonal only.

Bounds.  Symmetry, the sum and the row sums: SAME = 1e-9 kJ/mol, absolute -- the scale on which
tests/test_binding_decomposition_restatement.py holds sum D to u (each member's terms sum to its oracle energy within that).
Receptor x ligand cells: exact, because the sub-systems' matrices have an exact 0.0 there (a set that is empty in a member
receives no term at all)."""
import os

import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from tests.binding_decomposition_restatement import restate as restate_terms
from tests.binding_pair_matrix_restatement import restate, restate_members
from tests.binding_restatement import restate as restate_binding

SAME = 1e-9
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _residues(name):
    sets, labels = P.load_sets(os.path.join(GOLDEN, f"residues_{name}.txt"))
    return np.asarray(sets), len(labels)


def _cases():
    sets, S = _residues("trpcage")
    return {
        "trpcage_0_15_residues": ("trpcage", list(range(0, 16)), sets, S),          # the ligand cuts residues: mixed sets
        "trpcage_0_15_straddling": ("trpcage", list(range(0, 16)), "straddling", 18),  # (i + 8) // 16: a set wholly in the ligand
        "trpcage_every_third_mod3": ("trpcage", list(range(0, 272, 3)), None, 3),     # (None: i % 3)
    }


CASES = _cases()
RESULTS = {}


def _result(name):
    """(system, ligand, sets, S, D, u, members) of a case, computed once."""
    if name not in RESULTS:
        system, ligand, sets, S = CASES[name]
        s = P.load_system(system)
        sets = np.arange(s.n) % 3 if sets is None else (np.arange(s.n) + 8) // 16 if isinstance(sets, str) else sets
        assert len(sets) == s.n
        d, u, members = restate_members(s.params(), ligand, s.pos, sets, S)
        RESULTS[name] = (s, ligand, sets, S, d, u, members)
    return RESULTS[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_symmetric_and_sums_to_the_binding_energy(name):
    s, ligand, sets, S, d, u, _ = _result(name)
    u_ref = restate_binding(s.params(), ligand, s.pos, 0.35, version=1)[1]
    print(f"{name}: u = {u_ref!r}, |sum D - u| = {abs(d.sum() - u_ref):.3e}, asymmetry {np.abs(d - d.T).max():.3e}")
    assert d.shape == (S, S) and np.isfinite(d).all()
    assert u == u_ref
    assert np.abs(d - d.T).max() < SAME
    assert abs(d.sum() - u_ref) < SAME
    d2, u2 = restate(s.params(), ligand, s.pos, sets, S)  # (the two-result form is the same computation)
    assert np.array_equal(d2, d) and u2 == u


@pytest.mark.parametrize("name", sorted(CASES))
def test_rows_sum_to_the_sets_shares_of_the_per_atom_decomposition(name):
    s, ligand, sets, S, d, _, _ = _result(name)
    terms, _ = restate_terms(s.params(), ligand, s.pos, version=1)
    shares = np.zeros(S)
    np.add.at(shares, sets, terms.sum(axis=0))
    worst = np.abs(d.sum(axis=1) - shares).max()
    print(f"{name}: worst |row sum - share| = {worst:.3e}")
    assert worst < SAME


@pytest.mark.parametrize("name", sorted(CASES))
def test_receptor_by_ligand_cells_are_the_complexes_own(name):
    s, ligand, sets, S, d, _, (m_rl, m_r, m_l) = _result(name)
    is_ligand = np.zeros(s.n, dtype=bool)
    is_ligand[ligand] = True
    in_ligand = np.array([is_ligand[sets == a].all() and (sets == a).any() for a in range(S)])
    in_receptor = np.array([(~is_ligand[sets == a]).all() and (sets == a).any() for a in range(S)])
    mixed = [a for a in range(S) if (sets == a).any() and not in_ligand[a] and not in_receptor[a]]
    print(f"{name}: {in_receptor.sum()} receptor sets, {in_ligand.sum()} ligand sets, mixed {mixed}")
    # atoms 0..15 cut the first two residues: two mixed sets, none wholly in the ligand; with the straddling partition atoms
    # 0..7 are a ligand set and 8..23 a mixed one; every third atom with i % 3: set 0 IS the ligand, sets 1 and 2 the receptor
    expected = {"trpcage_0_15_residues": (2, 0), "trpcage_0_15_straddling": (1, 1), "trpcage_every_third_mod3": (0, 1)}
    assert (len(mixed), int(in_ligand.sum())) == expected[name]
    block, other = np.ix_(in_receptor, in_ligand), np.ix_(in_ligand, in_receptor)
    assert np.array_equal(d[block], m_rl[block]) and np.array_equal(d[other], m_rl[other])
    assert (m_r[block] == 0.0).all() and (m_l[block] == 0.0).all()
    if expected[name][1]:
        assert d[block].all()  # (the cells are there: every receptor set meets the ligand set through the GB pair term)


def test_version_0_fills_the_diagonal_only():
    s = P.load_system("fixture264")
    ligand = list(range(200, 264))
    sets, S = (np.arange(s.n) + 8) // 16, (s.n + 7) // 16 + 1
    d, u = restate(s.params(), ligand, s.pos, sets, S, version=0)
    u_ref = restate_binding(s.params(), ligand, s.pos, 0.35, version=0)[1]
    print(f"version 0: u = {u!r}, trace D = {np.trace(d)!r}")
    assert u == u_ref
    assert (d - np.diag(np.diag(d)) == 0.0).all() and d.any()
    assert abs(np.trace(d) - u) < SAME
