"""The premise of the perturbation energies (include/agbnp_hip.h, agbnp_hip_perturbed_energies_*), pinned without a device: the
energy under another set of (gamma, vdw_alpha, charge) is an explicit function of that set over quantities that depend on the
geometry and the radii alone.  tests/perturbation_restatement.py's restate() -- ONE base oracle's self volumes and Born radii,
then the formula -- equals the oracle created with each set, within SAME (1e-9, scaled as energy_close scales it)."""
import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from tests.gpu_helpers import SAME, energy_close
from tests.perturbation_restatement import oracle_energies, restate, standard_sets


@pytest.mark.parametrize("cutoff", [None, 1.0])
@pytest.mark.parametrize("version", [0, 1])
@pytest.mark.parametrize("name", ["trpcage", "fixture264"])
def test_the_restatement_equals_the_oracle_of_every_set(name, version, cutoff):
    s = P.load_system(name)
    sets = standard_sets(s.params())
    own, energies = restate(s.params(), sets, s.pos, version=version, cutoff=cutoff)
    reference = oracle_energies(s.params(), sets, s.pos, version=version, cutoff=cutoff)
    print(name, version, cutoff, "worst |restatement - oracle|", np.abs(energies - reference).max())
    for e, eo in zip(energies, reference):
        energy_close(e, eo, tol=SAME)
    # the base oracle's own parameters as a set: the formula gives back its own energy
    energy_close(restate(s.params(), [tuple(s.params()[1:4])], s.pos, version=version, cutoff=cutoff)[1][0], own, tol=SAME)
    if version == 1:
        assert len({round(float(e), 6) for e in reference}) == len(reference)  # (four different questions)


def test_a_hydrogens_gamma_counts_as_zero():
    s = P.load_system("trpcage")
    radius, gamma, alpha, charge, ish = [np.asarray(p, dtype=np.float64) for p in s.params()]
    loud = np.where(ish != 0, 123.0, gamma)  # gammas on the hydrogens, which no energy may see
    _, e = restate(s.params(), [(gamma, alpha, charge), (loud, alpha, charge)], s.pos)
    assert e[0] == e[1]
