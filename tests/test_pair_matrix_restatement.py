"""Set-pair interaction matrices (include/agbnp_hip.h: agbnp_hip_pair_matrix_*): the reference of the device tests and the
residue fixtures, at the boundaries that need no device.

The identities of tests/pair_matrix_restatement.py: the matrix is symmetric; it sums to the energy Oracle.execute() returns and
its rows to the per-set sums of the four per-atom terms, within SAME (1e-9 kJ/mol: the same FP64 numbers added in another order);
with every atom its own set the off-diagonal is the bare pair matrix k q_i q_j f_ij.  That makes it a reference the device's S S
entries can be compared with one by one (tests/test_gpu_pair_matrix.py).

The fixtures tests/golden/residues_*.txt (written by tests/golden/make_residue_fixtures.py): one line per atom in the order of the
bundled structures, 20 residues for trpcage -- one of them NOT contiguous in atom order -- and 258 for 1dwc."""
import os

import numpy as np

import openmm_agbnp_plugin_amd as P
from tests.decomposition_restatement import DIEL, restate
from tests.gpu_helpers import SAME
from tests.pair_matrix_restatement import restate_matrix

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RESIDUES = {"trpcage": (272, 20), "1dwc": (4152, 258)}


def runs(sets):
    return 1 + int(np.count_nonzero(np.diff(sets)))


def test_the_residue_fixtures_load_in_the_order_of_the_structures():
    for name, (atoms, residues) in RESIDUES.items():
        sets, labels = P.load_sets(os.path.join(GOLDEN, f"residues_{name}.txt"))
        assert sets.dtype == np.int32 and sets.shape == (atoms,) == (P.load_system(name).n,)
        assert len(labels) == residues == len(set(labels)) and sorted(set(sets.tolist())) == list(range(residues))
        assert all(len(label.split()) == 3 for label in labels)  # resid chain resname
        # the sets are numbered as the file first names them
        first = [int(np.flatnonzero(sets == k)[0]) for k in range(residues)]
        assert first == sorted(first)
        # the same atom order as the committed .dms fixtures: a hydrogen there is a hydrogen here, charge by charge
        dms = P.load_dms(os.path.join(GOLDEN, f"{name}_agbnp1.dms"))
        s = P.load_system(name)
        assert np.array_equal(dms.ishydrogen, s.ishydrogen) and np.abs(dms.charge - s.charge).max() < 1e-12
    assert labels[0] == "30 H ILE"


def test_one_trpcage_residue_is_not_contiguous():
    sets, labels = P.load_sets(os.path.join(GOLDEN, "residues_trpcage.txt"))
    assert runs(sets) == 21 > len(labels)
    assert sets[0] == sets[-1] == 0 and labels[0] == "1 A ASP"  # (the N terminus' hydrogens close the file)
    sets_1dwc, labels_1dwc = P.load_sets(os.path.join(GOLDEN, "residues_1dwc.txt"))
    assert runs(sets_1dwc) == len(labels_1dwc)


def test_the_restatement_on_trpcage_residues_is_symmetric_and_sums_to_the_energy():
    s = P.load_system("trpcage")
    sets, labels = P.load_sets(os.path.join(GOLDEN, "residues_trpcage.txt"))
    energy, matrix, terms = restate_matrix(s.params(), s.pos, sets, len(labels))
    assert matrix.shape == (20, 20) and np.isfinite(matrix).all()
    per_set = np.zeros(len(labels))
    np.add.at(per_set, sets, terms.sum(axis=0))
    figures = dict(symmetry=np.abs(matrix - matrix.T).max(), total=abs(matrix.sum() - energy),
                   rows=np.abs(matrix.sum(axis=1) - per_set).max())
    print(figures)
    for what, err in figures.items():
        assert err < SAME, f"{what}: {err:.3e}"
    assert np.abs(matrix - np.diag(np.diag(matrix))).max() > 1.0  # kJ/mol: residues do interact


def test_with_a_cutoff_the_matrix_sums_to_the_cutoff_energy():
    s = P.load_system("trpcage")
    sets, labels = P.load_sets(os.path.join(GOLDEN, "residues_trpcage.txt"))
    energy, matrix, terms = restate_matrix(s.params(), s.pos, sets, len(labels), cutoff=1.0)
    full = restate_matrix(s.params(), s.pos, sets, len(labels))[1]
    assert abs(matrix.sum() - energy) < SAME and np.abs(matrix - matrix.T).max() < SAME
    assert np.abs(matrix - full).max() > 1e-3  # (the cutoff truncates pairs, and the Born radii are other ones)


def test_every_atom_its_own_set_gives_the_bare_pair_matrix():
    s = P.load_system("fixture264")
    energy, matrix, terms = restate_matrix(s.params(), s.pos, np.arange(s.n), s.n)
    o = restate(s.params(), s.pos)[2]
    born, q = o.vector("born"), s.charge
    worst = 0.0
    rng = np.random.default_rng(7)
    for i, j in rng.integers(0, s.n, (200, 2)):
        if i == j:
            continue
        d2 = ((s.pos[i] - s.pos[j]) ** 2).sum()
        bb = born[i] * born[j]
        worst = max(worst, abs(matrix[i, j] - DIEL * q[i] * q[j] / np.sqrt(d2 + bb * np.exp(-0.25 * d2 / bb))))
    assert worst < 1e-12
    assert np.abs(np.diag(matrix) - terms[:3].sum(axis=0)).max() < 1e-12  # (no pair inside a set of one)
    assert abs(matrix.sum() - energy) < SAME


def test_version_0_fills_the_diagonal_only_and_empty_sets_stay_zero():
    s = P.load_system("fixture264")
    sets = 2 * (np.arange(s.n) // 16)
    energy, matrix, _ = restate_matrix(s.params(), s.pos, sets, 2 * ((s.n + 15) // 16), version=0)
    assert abs(np.trace(matrix) - energy) < SAME and (matrix - np.diag(np.diag(matrix)) == 0.0).all()
    _, full, _ = restate_matrix(s.params(), s.pos, sets, 2 * ((s.n + 15) // 16))
    assert (full[1::2] == 0.0).all() and (full[:, 1::2] == 0.0).all() and np.abs(np.diag(full)[::2]).min() > 0.0
