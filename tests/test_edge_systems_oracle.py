"""CPU: pins the inputs of tests/test_gpu_edge_regimes.py (tests/edge_systems.py) with the oracle, so that the GPU tests cannot
silently stop reaching their regime: the Born radii of born_clamp ARE at the 2 nm cap of ReferenceAGBNPKernels.cpp:41-55 (and one
is between 1 and 2 nm, and an atom crosses beta = 0 between jittered geometries), every system stays on the smallest store (no
capacity negotiation in front of the evaluations the GPU tests compare), the energies are the recorded ones, and the host I4
tables of its radius types (0.30 and 0.15 nm reach integral branches of AGBNPUtils.cpp:42-69 that the protein radii do not)
are the oracle's."""
import numpy as np
import pytest

import openmm_agbnp_plugin_amd as P
from oracle import Oracle
from tests.edge_systems import NAMES, ORACLE_ENERGY, SIZE_EDGES, STRIP_GAPS, STRIP_NAMES, block_gap, edge_systems, size_edge_name

SMALLEST_STORE = 432  # nodes of a subtree that the smallest LDS store holds
CAP = 2.0             # nm: kI4MaxA, the Born radius of beta < 0


def _born(s, pos=None, **kw):
    o = Oracle(*s.params(), version=1, **kw)
    o.execute(s.pos if pos is None else pos)
    return o.vector("born")


def test_the_table_is_what_the_gpu_tests_parametrise_over():
    table = edge_systems()
    assert tuple(table) == NAMES and len(set(NAMES)) == len(NAMES)
    for nh, n in SIZE_EDGES:
        s = table[size_edge_name(nh, n)]
        assert (s.nheavy, s.n) == (nh, n)
    assert table["born_clamp"].n == 21 and table["born_clamp"].nheavy == 9


def test_born_clamp_reaches_the_cap_and_the_arm_below_it():
    s = edge_systems()["born_clamp"]
    born = _born(s)
    capped = born == CAP
    assert capped.sum() >= 8
    assert (capped & (s.ishydrogen == 0)).any(), "no heavy atom at the cap"
    assert ((born > 1.0) & (born < CAP)).any()
    assert born.max() == CAP
    pos = s.pos
    dist = np.linalg.norm(pos[:, None] - pos[None], axis=-1)[np.triu_indices(s.n, 1)]
    assert dist.min() > 0.05  # (no two atoms on top of each other: the forces stay below a protein's)


def test_an_atom_crosses_the_cap_between_jittered_geometries():
    s = edge_systems()["born_clamp"]
    counts = [int((_born(s, s.jittered(step)) == CAP).sum()) for step in range(4)]
    assert min(counts) >= 8 and len(set(counts)) >= 2, counts


def test_the_cutoff_oracle_keeps_a_capped_atom_at_the_long_cutoff():
    s = edge_systems()["born_clamp"]
    assert (_born(s, cutoff=1.2) == CAP).sum() >= 1


@pytest.mark.parametrize("name", list(ORACLE_ENERGY))
def test_recorded_energies_of_the_born_clamp_family(name):
    s = edge_systems()[name]
    o = Oracle(*s.params(), version=1)
    e, f = o.execute(s.pos)
    assert abs(e - ORACLE_ENERGY[name]) <= 1e-9 * abs(ORACLE_ENERGY[name])
    assert o.tree_stats()["max_subtree"] <= SMALLEST_STORE
    if name == "born_clamp_q0":
        assert o.scalar("e_gb") == 0.0
    if name == "born_clamp":  # central differences of the energy reproduce the forces
        h = 1e-5
        for atom, d in ((8, 0), (0, 1), (13, 2)):
            pp, pm = s.pos.copy(), s.pos.copy()
            pp[atom, d] += h
            pm[atom, d] -= h
            assert abs(-(o.execute(pp)[0] - o.execute(pm)[0]) / (2 * h) - f[atom, d]) < 1e-5 * max(1.0, abs(f[atom, d]))


@pytest.mark.parametrize("name", STRIP_NAMES)
def test_the_three_block_systems_straddle_the_far_strip_bound(name):
    """Blocks 0 and 1 against block 2: capped Born radii on both sides; the boxes' gaps are 12 nm (beyond the bound of Born radii
    under 0.93 nm, far inside that of capped ones) and either side of sqrt(4 * 60 ln2 * 2 * 2) nm, on the file geometry and on the
    jittered one that the GPU test evaluates."""
    s = edge_systems()[name]
    assert s.n == 149 and (s.n + 63) // 64 == 3
    born = _born(s)
    assert all((born[64 * b: 64 * b + 64] == CAP).any() for b in range(3))
    bound = float(np.sqrt(4.0 * 60.0 * np.log(2.0) * CAP * CAP))
    assert 25.7 < bound < 25.9 and STRIP_GAPS[1] < bound - 1.0 and STRIP_GAPS[2] > bound + 1.0
    assert np.sqrt(4.0 * 60.0 * np.log(2.0) * 0.93 * 0.93) < STRIP_GAPS[0] < bound / 2
    want = STRIP_GAPS[STRIP_NAMES.index(name)]
    for pos in (s.pos, s.jittered(5, sigma=0.003)):
        assert abs(block_gap(s, pos) - want) < 0.05
    o = Oracle(*s.params(), version=1)
    assert np.isfinite(o.execute(s.pos)[0]) and o.tree_stats()["max_subtree"] <= SMALLEST_STORE


@pytest.mark.parametrize("version", [0, 1])
@pytest.mark.parametrize("nh,n", SIZE_EDGES)
def test_size_edges_stay_on_the_smallest_store(nh, n, version):
    s = edge_systems()[size_edge_name(nh, n)]
    o = Oracle(*s.params(), version=version)
    e, f = o.execute(s.pos)
    assert np.isfinite(e) and np.isfinite(f).all()
    assert o.tree_stats()["max_subtree"] <= SMALLEST_STORE
    if version == 1:
        assert o.vector("born").max() < 1.0  # (the size edges are ordinary protein pieces: the cap is born_clamp's business)


def test_host_i4_tables_of_the_born_clamp_radii_match_the_oracle():
    """Compared the way tests/test_host_api.py::test_host_i4_tables_match_oracle does it."""
    s = edge_systems()["born_clamp"]
    t = P.host_tables(s.radius, s.ishydrogen)
    o = Oracle(*s.params(), version=1).tables()
    assert t["y"].shape == o["y"].shape == (3, 2, 16)
    np.testing.assert_array_equal(t["type_screened"], o["type_screened"])
    np.testing.assert_array_equal(t["type_screener"], o["type_screener"])
    np.testing.assert_allclose(t["y"], o["y"], rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(t["y2"], o["y2"], rtol=1e-11, atol=1e-13)
    assert np.abs(t["y"][:, :, -1]).max() < 1e-12
